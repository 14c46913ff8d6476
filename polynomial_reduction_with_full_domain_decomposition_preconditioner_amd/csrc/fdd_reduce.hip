// Dot-product style reductions (HBM-bound): the four Domain dot kernels
// (domain.okl:109-264), the Subdomain ones (subdomain.okl:103-258) and the
// cublasDdot replacement of AMG/vector.cpp.
//
// The reference writes one partial per 128-thread block, copies all of them to
// the host (131 072 doubles at config C2) and sums them there.  Here a capped
// grid (<= 2048 workgroups) strides over the vectors with 16-B loads, each
// lane keeps a private sum, a wavefront __shfl_down tree and a 4-wave LDS step
// give one partial per workgroup, and a second one-workgroup launch folds the
// partials into the final scalar on the device.  The result is deterministic
// for a given n (fixed grid, fixed tree) but its summation order differs from
// the reference's 128-wide tree + serial block sum: parity is
// tolerance-based (tests/).
//
// Every op states its terms once, in at(), over a lane accessor (fdd_stream.h): a
// pair adds its first element's term and then its second's to the lane's sum.
#include "fdd_stream.h"

namespace
{

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / FDD_WAVE;
using Single = fdd_lanes<1>;
using Pair = fdd_lanes<2>;

// NV values per element (1 or 2 simultaneous sums)
template <int NV>
struct Acc
{
    double v[NV];
};

template <int NV>
__device__ __forceinline__ void block_reduce_store(Acc<NV> a, double *ws, int nblocks_stride)
{
    __shared__ double s[NV][kWaves];
    const int lane = threadIdx.x & (FDD_WAVE - 1);
    const int wave = threadIdx.x / FDD_WAVE;

#pragma unroll
    for (int k = 0; k < NV; k++)
    {
        double x = wave_sum(a.v[k]);
        if (lane == 0) s[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
#pragma unroll
        for (int k = 0; k < NV; k++)
        {
            double x = s[k][0];
#pragma unroll
            for (int w = 1; w < kWaves; w++) x += s[k][w];
            ws[blockIdx.x + k * nblocks_stride] = x;
        }
    }
}

// the three kernels' bodies, stated once for the plain launches and for the gated ones below
template <typename Op>
__device__ __forceinline__ void reduce_vec2_body(const Op &op, double *ws, long long n2, long long n)
{
    Acc<Op::NV> a;
#pragma unroll
    for (int k = 0; k < Op::NV; k++) a.v[k] = 0.0;

    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n2; i += stride) op.at(Pair{}, i, a);
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) op.at(Single{}, n - 1, a);

    block_reduce_store<Op::NV>(a, ws, FDD_REDUCE_MAX_BLOCKS);
}

template <typename Op>
__device__ __forceinline__ void reduce_scalar_body(const Op &op, double *ws, long long n)
{
    Acc<Op::NV> a;
#pragma unroll
    for (int k = 0; k < Op::NV; k++) a.v[k] = 0.0;

    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) op.at(Single{}, i, a);

    block_reduce_store<Op::NV>(a, ws, FDD_REDUCE_MAX_BLOCKS);
}

template <typename Op>
__global__ __launch_bounds__(kBlock) void reduce_vec2_kernel(Op op, double *ws, long long n2, long long n)
{
    reduce_vec2_body(op, ws, n2, n);
}

template <typename Op>
__global__ __launch_bounds__(kBlock) void reduce_scalar_kernel(Op op, double *ws, long long n)
{
    reduce_scalar_body(op, ws, n);
}

// Gate of the last Arnoldi step's exact norm pass (fdd_norm_estimate.h): dots[0..m-1] are the projections of this step and
// dots[m] the self product.  Where the norm may be taken from them the launch has nothing to do: every workgroup asks the same
// question of the same m + 1 numbers (wave-uniform) and returns before it reads a vector or writes anything.
__device__ __forceinline__ bool norm_pass_needed(const double *dots, int m)
{
    double est;
    return !fdd_norm2_from_projections(dots[m], dots, m, &est);
}

template <typename Op>
__global__ __launch_bounds__(kBlock) void reduce_vec2_gated_kernel(Op op, double *ws, long long n2, long long n, const double *dots, int m)
{
    if (!norm_pass_needed(dots, m)) return;
    reduce_vec2_body(op, ws, n2, n);
}

template <typename Op>
__global__ __launch_bounds__(kBlock) void reduce_scalar_gated_kernel(Op op, double *ws, long long n, const double *dots, int m)
{
    if (!norm_pass_needed(dots, m)) return;
    reduce_scalar_body(op, ws, n);
}

// second stage: one workgroup folds `nblocks` partials per value
template <int NV>
__device__ __forceinline__ void reduce_final_body(double *out, const double *ws, int nblocks);

template <int NV>
__global__ __launch_bounds__(kBlock) void reduce_final_kernel(double *out, const double *ws, int nblocks)
{
    reduce_final_body<NV>(out, ws, nblocks);
}

template <int NV>
__global__ __launch_bounds__(kBlock) void reduce_final_gated_kernel(double *out, const double *ws, int nblocks, const double *dots, int m)
{
    if (!norm_pass_needed(dots, m)) return;
    reduce_final_body<NV>(out, ws, nblocks);
}

template <int NV>
__device__ __forceinline__ void reduce_final_body(double *out, const double *ws, int nblocks)
{
    __shared__ double s[NV][kWaves];
    const int lane = threadIdx.x & (FDD_WAVE - 1);
    const int wave = threadIdx.x / FDD_WAVE;

    // every partial this lane folds is requested before the first one is added (one round trip to the partials the
    // previous launch left in memory instead of one per partial); the sums and their order are those of the plain loop
    constexpr int kPer = FDD_REDUCE_MAX_BLOCKS / kBlock;
    double v[NV][kPer];
#pragma unroll
    for (int k = 0; k < NV; k++)
#pragma unroll
        for (int i = 0; i < kPer; i++)
        {
            const int b = threadIdx.x + i * kBlock;
            v[k][i] = ws[(b < nblocks ? b : 0) + k * FDD_REDUCE_MAX_BLOCKS];
        }
#pragma unroll
    for (int k = 0; k < NV; k++)
    {
        double x = 0.0;
#pragma unroll
        for (int i = 0; i < kPer; i++)
            if (threadIdx.x + i * kBlock < nblocks) x += v[k][i];
        x = wave_sum(x);
        if (lane == 0) s[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
#pragma unroll
        for (int k = 0; k < NV; k++)
        {
            double x = s[k][0];
#pragma unroll
            for (int w = 1; w < kWaves; w++) x += s[k][w];
            out[k] = x;
        }
    }
}

template <typename Op>
int launch_reduce(const Op &op, double *out, double *ws, long long n, void *stream)
{
    hipStream_t s = fdd_stream(stream);
    if (n <= 0)
    {
        // empty sums are zero; keep it asynchronous
        return (int)hipMemsetAsync(out, 0, sizeof(double) * Op::NV, s);
    }

    int grid;
    if (fdd_lanes_fit<Pair>(op) && n >= 2)
    {
        long long n2 = n / 2;
        grid = fdd_stream_grid(n2, kBlock);
        hipLaunchKernelGGL(reduce_vec2_kernel<Op>, dim3(grid), dim3(kBlock), 0, s, op, ws, n2, n);
    }
    else
    {
        grid = fdd_stream_grid(n, kBlock);
        hipLaunchKernelGGL(reduce_scalar_kernel<Op>, dim3(grid), dim3(kBlock), 0, s, op, ws, n);
    }
    FDD_LAUNCH_CHECK();
    hipLaunchKernelGGL(reduce_final_kernel<Op::NV>, dim3(1), dim3(kBlock), 0, s, out, ws, grid);
    FDD_LAUNCH_CHECK();
    return 0;
}

// launch_reduce behind the gate of norm_pass_needed(dots, m): the same path, grid and fold, hence the same bits where the gate
// is open; where it is closed neither launch writes out, ws or anything the op stores.  An empty sum is the fold over no partials.
template <typename Op>
int launch_reduce_gated(const Op &op, double *out, double *ws, long long n, const double *dots, int m, void *stream)
{
    hipStream_t s = fdd_stream(stream);
    int grid = 0;
    if (n <= 0)
        ;
    else if (fdd_lanes_fit<Pair>(op) && n >= 2)
    {
        long long n2 = n / 2;
        grid = fdd_stream_grid(n2, kBlock);
        hipLaunchKernelGGL(reduce_vec2_gated_kernel<Op>, dim3(grid), dim3(kBlock), 0, s, op, ws, n2, n, dots, m);
    }
    else
    {
        grid = fdd_stream_grid(n, kBlock);
        hipLaunchKernelGGL(reduce_scalar_gated_kernel<Op>, dim3(grid), dim3(kBlock), 0, s, op, ws, n, dots, m);
    }
    FDD_LAUNCH_CHECK();
    hipLaunchKernelGGL(reduce_final_gated_kernel<Op::NV>, dim3(1), dim3(kBlock), 0, s, out, ws, grid, dots, m);
    FDD_LAUNCH_CHECK();
    return 0;
}

// Every op: at(l, i, acc) adds the terms of element i of accessor l to the lane's sums, pointers(f) names the vectors it touches.

struct Dot2Op // subdomain.okl:103-132 / cublasDdot
{
    static constexpr int NV = 1;
    const double *u, *v;
    template <typename A>
    __device__ void at(A l, long long i, Acc<1> &acc) const { l.add(acc.v[0], l.ld(u, i) * l.ld(v, i)); }
    template <typename F>
    void pointers(F f) const { f(u), f(v); }
};

struct Dot3Op // domain.okl:109-138 (r*QQt_r*mask), :235-264 (u*v*mask), subdomain.okl:134-163 (u*v*w)
{
    static constexpr int NV = 1;
    const double *u, *v, *w;
    template <typename A>
    __device__ void at(A l, long long i, Acc<1> &acc) const { l.add(acc.v[0], l.ld(u, i) * l.ld(v, i) * l.ld(w, i)); }
    template <typename F>
    void pointers(F f) const { f(u), f(v), f(w); }
};

struct ProjOp // domain.okl:140-184
{
    static constexpr int NV = 2;
    const double *z, *r, *p, *q;
    template <typename A>
    __device__ void at(A l, long long i, Acc<2> &acc) const
    {
        const auto zz = l.ld(z, i), rr = l.ld(r, i), pp = l.ld(p, i), qq = l.ld(q, i);
        l.add(acc.v[0], zz * rr);
        l.add(acc.v[1], pp * qq);
    }
    template <typename F>
    void pointers(F f) const { f(z), f(r), f(p), f(q); }
};

struct ProjWOp // subdomain.okl:165-209
{
    static constexpr int NV = 2;
    const double *z, *r, *p, *q, *w;
    template <typename A>
    __device__ void at(A l, long long i, Acc<2> &acc) const
    {
        const auto zz = l.ld(z, i), rr = l.ld(r, i), pp = l.ld(p, i), qq = l.ld(q, i), ww = l.ld(w, i);
        l.add(acc.v[0], zz * rr * ww);
        l.add(acc.v[1], pp * qq * ww);
    }
    template <typename F>
    void pointers(F f) const { f(z), f(r), f(p), f(q), f(w); }
};

struct FlexOp // domain.okl:195-224
{
    static constexpr int NV = 1;
    const double *r, *r1, *z;
    template <typename A>
    __device__ void at(A l, long long i, Acc<1> &acc) const
    {
        const auto a0 = l.ld(r, i), a1 = l.ld(r1, i), zz = l.ld(z, i);
        l.add(acc.v[0], (a1 - a0) * zz);
    }
    template <typename F>
    void pointers(F f) const { f(r), f(r1), f(z); }
};

// the flexible dot and, from the same three streams, the NEXT iteration's gamma = <z, r+> (domain.okl:140-184's first sum one
// iteration early: the projection kernel of that iteration is then left with <p, q> alone).  out = {gamma_next, theta}.
struct FlexGammaOp
{
    static constexpr int NV = 2;
    const double *r, *r1, *z;
    // the two sums' terms, given the values of r, r+ and z
    template <typename A, typename V>
    static __device__ __forceinline__ void add(A l, Acc<2> &acc, V a0, V a1, V zz)
    {
        l.add(acc.v[0], zz * a1);
        l.add(acc.v[1], (a1 - a0) * zz);
    }
    template <typename A>
    __device__ void at(A l, long long i, Acc<2> &acc) const { add(l, acc, l.ld(r, i), l.ld(r1, i), l.ld(z, i)); }
    template <typename F>
    void pointers(F f) const { f(r), f(r1), f(z); }
};

// FlexGammaOp with z's slice [lo, hi) not read but FORMED on the way: z[i] = (z[i] or 0) + sum_{k <= *last} c_k (vs_k v_k[i - lo]),
// the statement of MultiAxpyDevOp (fdd_blas1.hip; fdd_lincomb, fdd_stream.h), stored, and entered into the two sums where
// the stored value would have been loaded.  The traversal (pairs, accumulators, expressions, their order) is FlexGammaOp's,
// so z and both sums have the bits of fdd_multi_lincomb_limited_dev followed by fdd_dom_inner_product_flexible_gamma --
// without writing z and reading it back, and, where v_0 is r1's own slice (the inner solve's right-hand side read in place),
// without reading that twice.  A pair can lie astride a slice end, so the two accessors have a body each here.
template <int M>
struct LincombFlexGammaOp
{
    static constexpr int NV = 2;
    const double *r, *r1;
    double *z;
    long long lo, hi;
    const double *v[M]; // v[k][i - lo] belongs to node i
    const double *c;
    const double *vs;   // optional per-vector scales
    const double *last; // optional: only vectors 0..(int)*last enter
    bool from_zero;     // z's slice is taken as 0 and not read
    bool v0_is_r1;      // v[0] == r1 + lo: its entries are the ones this pass loads from r1 anyway
    bool v_pairs;       // lo is even and every v[k] is aligned for pairs: a pair inside the slice is one 16-byte load per vector

    __device__ __forceinline__ int kmax() const { return last ? (int)*last : M - 1; }
    __device__ __forceinline__ double form(long long i, double r1_i, int kmax) const
    {
        const double x = fdd_lincomb<M>(from_zero ? 0.0 : z[i], kmax, c, vs, [&](int k) { return (k == 0 && v0_is_r1) ? r1_i : v[k][i - lo]; });
        z[i] = x;
        return x;
    }
    __device__ void at(Pair l, long long i, Acc<2> &acc) const
    {
        using V = Pair::value<double>;
        const V a0 = l.ld(r, i), a1 = l.ld(r1, i);
        const long long g = 2 * i;
        const bool in0 = g >= lo && g < hi, in1 = g + 1 >= lo && g + 1 < hi;
        V zz;
        if (in0 && in1)
        {
            zz = fdd_lincomb<M>(from_zero ? l.all(0.0) : l.ld(z, i), kmax(), c, vs, [&](int k) -> V {
                if (k == 0 && v0_is_r1) return a1;
                if (v_pairs) return l.ld(v[k], (g - lo) >> 1);
                return {__builtin_nontemporal_load(v[k] + (g - lo)), __builtin_nontemporal_load(v[k] + (g - lo) + 1)};
            });
            l.st(z, i, zz); // default policy: the direction update reads it next
        }
        else if (in0 || in1) // a pair astride a slice end: per component
        {
            const int km = kmax();
            zz.c[0] = in0 ? form(g, a1.c[0], km) : z[g];
            zz.c[1] = in1 ? form(g + 1, a1.c[1], km) : z[g + 1];
        }
        else
            zz = l.ld(z, i);
        FlexGammaOp::add(l, acc, a0, a1, zz);
    }
    __device__ void at(Single l, long long i, Acc<2> &acc) const
    {
        const double r1_i = r1[i];
        FlexGammaOp::add(l, acc, r[i], r1_i, (i >= lo && i < hi) ? form(i, r1_i, kmax()) : z[i]);
    }
    // the same selection as fdd_dom_inner_product_flexible_gamma's: the pairing of the sums is that entry's
    template <typename F>
    void pointers(F f) const { f(r), f(r1), f(z); }
};

template <int M>
int launch_lincomb_flex_gamma(double *out2, double *ws, const double *r, const double *r1, double *z, int n, int lo, int nd, bool from_zero, const double *c, const double *const *v, const double *vs, const double *last, void *stream)
{
    LincombFlexGammaOp<M> op;
    op.r = r;
    op.r1 = r1;
    op.z = z;
    op.lo = lo;
    op.hi = (long long)lo + nd;
    op.c = c;
    op.vs = vs;
    op.last = last;
    op.from_zero = from_zero;
    op.v0_is_r1 = v[0] == r1 + lo;
    op.v_pairs = (lo & 1) == 0;
    for (int k = 0; k < M; k++)
    {
        op.v[k] = v[k];
        op.v_pairs = op.v_pairs && fdd_aligned(v[k], Pair::bytes<double>);
    }
    return launch_reduce(op, out2, ws, n, stream);
}

struct FlexWOp // subdomain.okl:229-258
{
    static constexpr int NV = 1;
    const double *r, *r1, *z, *w;
    template <typename A>
    __device__ void at(A l, long long i, Acc<1> &acc) const
    {
        const auto a0 = l.ld(r, i), a1 = l.ld(r1, i), zz = l.ld(z, i), ww = l.ld(w, i);
        l.add(acc.v[0], (a1 - a0) * zz * ww);
    }
    template <typename F>
    void pointers(F f) const { f(r), f(r1), f(z), f(w); }
};

// out[i] = sum a * b_i * w for i < M: `a` and `w` are read once for all M dots
// (the reference launches weighted_inner_product once per pair, subdomain.tpp:4389-4394)
// the terms of element i, for MultiDotWOp<M> (NV = M) and MultiDotSelfOp<M> (NV = M + 1: the self product sum a*a*w behind
// them, from the values already loaded; it takes no scale)
template <int M, int NV, typename A>
__device__ __forceinline__ void multi_dot_at(A l, long long i, const double *a, const double *w, const double *const (&b)[M], const double *bs, Acc<NV> &acc)
{
    const auto aa = l.ld(a, i), ww = w ? l.ld(w, i) : l.all(1.0); // w == NULL: unit weights, not read (x * 1.0 is x)
#pragma unroll
    for (int k = 0; k < M; k++)
    {
        auto bb = (b[k] == a) ? aa : l.ld(b[k], i); // <a, a>: one stream, not two
        if (bs) bb = bs[k] * bb;
        l.add(acc.v[k], aa * bb * ww);
    }
    if constexpr (NV > M) l.add(acc.v[M], aa * aa * ww);
}

template <int M>
struct MultiDotWOp
{
    static constexpr int NV = M;
    const double *a, *w;
    const double *b[M];
    const double *bs; // optional: b_k stands for bs[k] * b_k (a Krylov basis kept unnormalised, its 1/norm on the device)
    template <typename A>
    __device__ void at(A l, long long i, Acc<M> &acc) const
    {
        multi_dot_at<M>(l, i, a, w, b, bs, acc);
    }
    template <typename F>
    void pointers(F f) const
    {
        f(a), f(w);
        for (int k = 0; k < M; k++) f(b[k]);
    }
};

// MultiDotWOp<M> with out[M] = sum a*a*w: the traversal, and so the bits of the first M sums, are MultiDotWOp<M>'s
template <int M>
struct MultiDotSelfOp : MultiDotWOp<M>
{
    static constexpr int NV = M + 1;
    template <typename A>
    __device__ void at(A l, long long i, Acc<M + 1> &acc) const
    {
        multi_dot_at<M>(l, i, this->a, this->w, this->b, this->bs, acc);
    }
};

template <int M>
int launch_multi_dot(double *out, double *ws, const double *a, const double *const *b, const double *b_scale_dev, const double *w, int n, void *stream)
{
    MultiDotWOp<M> op;
    op.a = a;
    op.w = w;
    op.bs = b_scale_dev;
    for (int k = 0; k < M; k++) op.b[k] = b[k];
    return launch_reduce(op, out, ws, n, stream);
}

template <int M>
int launch_multi_dot_self(double *out, double *ws, const double *a, const double *const *b, const double *b_scale_dev, const double *w, int n, void *stream)
{
    MultiDotSelfOp<M> op;
    op.a = a;
    op.w = w;
    op.bs = b_scale_dev;
    for (int k = 0; k < M; k++) op.b[k] = b[k];
    return launch_reduce(op, out, ws, n, stream);
}

// Gram-Schmidt update and the norm of its result in one pass:
// y += sign * sum_k c[k] * x_k (the arithmetic of fdd_multi_axpy), out = sum y*y*w.
// The coefficients stay on the device (the output of fdd_multi_weighted_inner_product).
template <int M>
struct MultiAxpyNormOp
{
    static constexpr int NV = 1;
    double *dst;     // where the updated vector goes (y itself, or the next basis slot)
    const double *y;
    const double *w, *c;
    const double *x[M];
    const double *xs; // optional per-vector scales: x_k stands for xs[k] * x_k
    double sign;
    template <typename A>
    __device__ void at(A l, long long i, Acc<1> &acc) const
    {
        auto yy = l.ld(y, i);
        const auto ww = w ? l.ld(w, i) : l.all(1.0);
#pragma unroll
        for (int k = 0; k < M; k++)
        {
            const double ck = sign * c[k];
            auto b = l.ld(x[k], i);
            if (xs) b = xs[k] * b;
            yy = 1.0 * yy + ck * b;
        }
        if (dst) l.st(dst, i, yy); // dst == NULL: only the norm is wanted (the last Arnoldi step of a cycle)
        l.add(acc.v[0], yy * yy * ww);
    }
    template <typename F>
    void pointers(F f) const
    {
        f(y), f(w), f(dst);
        for (int k = 0; k < M; k++) f(x[k]);
    }
};

// gate_dots: NULL, or the M + 1 dots the launch is gated on (launch_reduce_gated)
template <int M>
int launch_multi_axpy_norm(double *out, double *ws, double *dst, const double *y, const double *c, double sign, const double *const *x, const double *x_scale_dev, const double *w, int n, void *stream, const double *gate_dots = nullptr)
{
    MultiAxpyNormOp<M> op;
    op.dst = dst;
    op.y = y;
    op.w = w;
    op.c = c;
    op.xs = x_scale_dev;
    op.sign = sign;
    for (int k = 0; k < M; k++) op.x[k] = x[k];
    if (gate_dots) return launch_reduce_gated(op, out, ws, n, gate_dots, M, stream);
    return launch_reduce(op, out, ws, n, stream);
}

// r1 = r - (*num / *den) * q over all n nodes (UpdateUROp's residual statement, fdd_blas1.hip) and, of the values it stores,
// the sum of squares over the slice [lo, lo + nd): MultiDotWOp<1> with b[0] == a and unit weights on r1 + lo, without
// reading r1 back.  Unlike LincombFlexGammaOp, whose pairs are the whole vector's, the traversal here is the SLICE's: the
// sum has the bits of launch_reduce(MultiDotWOp<1>{r1 + lo, ...}, nd) only if grid, path (pairs where r1 + lo is aligned
// for them and nd >= 2) and lane-to-element assignment are that launch's, counted from the slice start.  at() is the
// operation on element i of accessor l of the vectors `from` elements further on; it returns what it stored.
struct ResidualUpdateNormOp
{
    double *r1;
    const double *r, *q, *num, *den;
    template <typename A>
    __device__ typename A::template value<double> at(A l, long long from, long long i, bool wide_loads = true) const
    {
        const double al = num[0] / den[0];
        typename A::template value<double> rr, qq;
        if constexpr (std::is_same<A, Pair>::value)
        {
            if (wide_loads)
                rr = l.ld(r + from, i), qq = l.ld(q + from, i);
            else // r or q is not aligned for pairs where r1 is: the same two elements, loaded one by one
            {
                rr = {__builtin_nontemporal_load(r + from + 2 * i), __builtin_nontemporal_load(r + from + 2 * i + 1)};
                qq = {__builtin_nontemporal_load(q + from + 2 * i), __builtin_nontemporal_load(q + from + 2 * i + 1)};
            }
        }
        else
            rr = l.ld(r + from, i), qq = l.ld(q + from, i);
        const auto v = rr - al * qq;
        l.st(r1 + from, i, v);
        return v;
    }
    template <typename A, typename V>
    static __device__ __forceinline__ void add(A l, Acc<1> &acc, V v) { l.add(acc.v[0], v * v * l.all(1.0)); }
};

template <bool PAIRS>
__global__ __launch_bounds__(kBlock) void residual_update_norm_kernel(ResidualUpdateNormOp op, double *ws, long long lo, long long nd, long long n, bool wide_loads)
{
    Acc<1> a;
    a.v[0] = 0.0;
    const long long stride = (long long)gridDim.x * kBlock;
    const long long first = (long long)blockIdx.x * kBlock + threadIdx.x;
    // the slice, as reduce_vec2_kernel / reduce_scalar_kernel walk a vector that starts at lo
    if constexpr (PAIRS)
    {
        const long long nd2 = nd / 2;
        for (long long i = first; i < nd2; i += stride) ResidualUpdateNormOp::add(Pair{}, a, op.at(Pair{}, lo, i, wide_loads));
        if ((nd & 1) && first == 0) ResidualUpdateNormOp::add(Single{}, a, op.at(Single{}, lo, nd - 1));
    }
    else
        for (long long i = first; i < nd; i += stride) ResidualUpdateNormOp::add(Single{}, a, op.at(Single{}, lo, i));
    // the nodes in front of and behind the slice: updated, in no sum
    for (long long i = first; i < lo; i += stride) op.at(Single{}, 0, i);
    for (long long i = lo + nd + first; i < n; i += stride) op.at(Single{}, 0, i);

    block_reduce_store<1>(a, ws, FDD_REDUCE_MAX_BLOCKS);
}

// ||Qt_w u||^2 in one pass: per assembled node s = (sum_j 1.0*u[col_j]) * w,
// accumulate s*s*w -- the gather of multiply_weight (csr_matrix.okl:35-48) and
// the weighted_inner_product (subdomain.okl:134-163) of Subdomain::residual_norm
// (subdomain.tpp:4491-4515) without the intermediate dof vector.
__global__ __launch_bounds__(kBlock) void gather_norm2_kernel(double *ws, const int *__restrict__ Qt_ptr, const int *__restrict__ Qt_col, const double *__restrict__ u, const double *__restrict__ w, int n)
{
    Acc<1> a;
    a.v[0] = 0.0;
    constexpr int NPT = 4;
    const int stride = gridDim.x * kBlock * NPT;
    for (int tile = blockIdx.x * kBlock * NPT; tile < n; tile += stride)
    {
        int j0[NPT], j1[NPT];
        double wn[NPT], s[NPT];
#pragma unroll
        for (int r = 0; r < NPT; r++)
        {
            const int node = tile + r * kBlock + threadIdx.x;
            const bool on = node < n;
            j0[r] = on ? Qt_ptr[node] : 0;
            j1[r] = on ? Qt_ptr[node + 1] : 0;
            wn[r] = on ? w[node] : 0.0;
        }
        fdd_multi_row_sum<NPT, 4, true>(Qt_col, nullptr, u, j0, j1, s);
#pragma unroll
        for (int r = 0; r < NPT; r++)
        {
            const double sw = s[r] * wn[r];
            a.v[0] += sw * sw * wn[r];
        }
    }
    block_reduce_store<1>(a, ws, FDD_REDUCE_MAX_BLOCKS);
}

// ---------------------------------------------------------------------------------------------------------------
// Single-precision preconditioner (the reference's PTYPE = Float, config.hpp:19-20): the same two reductions on
// float vectors.  Storage is float; products and sums are carried in double (the partial sums of a 10^7-term float
// dot would lose half their digits in float), the Gram-Schmidt update is rounded to float where it is stored.
// ---------------------------------------------------------------------------------------------------------------
template <int M>
struct MultiDotOpF
{
    static constexpr int NV = M;
    const float *a;
    const float *b[M];
    const double *bs;
    template <typename A>
    __device__ void at(A l, long long i, Acc<M> &acc) const
    {
        const auto aa = l.ld(a, i);
#pragma unroll
        for (int k = 0; k < M; k++)
        {
            const auto bb = (b[k] == a) ? aa : l.ld(b[k], i);
            const double sk = bs ? bs[k] : 1.0;
            l.add(acc.v[k], A::template to<double>(aa) * (sk * A::template to<double>(bb)));
        }
    }
    template <typename F>
    void pointers(F f) const
    {
        f(a);
        for (int k = 0; k < M; k++) f(b[k]);
    }
};

template <int M>
int launch_multi_dot_f32(double *out, double *ws, const float *a, const float *const *b, const double *b_scale_dev, int n, void *stream)
{
    MultiDotOpF<M> op;
    op.a = a;
    op.bs = b_scale_dev;
    for (int k = 0; k < M; k++) op.b[k] = b[k];
    return launch_reduce(op, out, ws, n, stream);
}

template <int M>
struct MultiAxpyNormOpF
{
    static constexpr int NV = 1;
    float *dst;
    const float *y;
    const float *x[M];
    const double *c;  // coefficients on the device
    const double *xs; // optional scales of the x_k
    double sign;
    template <typename A>
    __device__ void at(A l, long long i, Acc<1> &acc) const
    {
        auto v = A::template to<double>(l.ld(y, i));
#pragma unroll
        for (int k = 0; k < M; k++)
        {
            const auto b = l.ld(x[k], i);
            const double ck = sign * c[k] * (xs ? xs[k] : 1.0);
            v = v + ck * A::template to<double>(b);
        }
        const auto rf = A::template to<float>(v);
        if (dst) l.st(dst, i, rf);
        const auto rd = A::template to<double>(rf);
        l.add(acc.v[0], rd * rd);
    }
    template <typename F>
    void pointers(F f) const
    {
        f(y), f(dst);
        for (int k = 0; k < M; k++) f(x[k]);
    }
};

template <int M>
int launch_multi_axpy_norm_f32(double *out, double *ws, float *dst, const float *y, const double *c, double sign, const float *const *x, const double *x_scale_dev, int n, void *stream)
{
    MultiAxpyNormOpF<M> op;
    op.dst = dst;
    op.y = y;
    op.c = c;
    op.xs = x_scale_dev;
    op.sign = sign;
    for (int k = 0; k < M; k++) op.x[k] = x[k];
    return launch_reduce(op, out, ws, n, stream);
}

} // namespace

extern "C" {

size_t fdd_reduce_workspace_doubles(void) { return FDD_MULTI_MAX * (size_t)FDD_REDUCE_MAX_BLOCKS; }

int fdd_dom_residual_norm(double *out, double *ws, const double *r_k, const double *QQt_r_k, const double *dirichlet_mask, int num_points, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && num_points >= 0);
    FDD_REQUIRE(num_points == 0 || (r_k != nullptr && QQt_r_k != nullptr && dirichlet_mask != nullptr));
    return launch_reduce(Dot3Op{r_k, QQt_r_k, dirichlet_mask}, out, ws, num_points, stream);
}

int fdd_dom_inner_product(double *out, double *ws, const double *u_k, const double *v_k, const double *dirichlet_mask, int num_points, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && num_points >= 0);
    FDD_REQUIRE(num_points == 0 || (u_k != nullptr && v_k != nullptr && dirichlet_mask != nullptr));
    return launch_reduce(Dot3Op{u_k, v_k, dirichlet_mask}, out, ws, num_points, stream);
}

int fdd_dom_projection_inner_products(double *out2, double *ws, const double *z_k, const double *r_k, const double *p_k, const double *q_k, int num_points, void *stream)
{
    FDD_REQUIRE(out2 != nullptr && ws != nullptr && num_points >= 0);
    FDD_REQUIRE(num_points == 0 || (z_k != nullptr && r_k != nullptr && p_k != nullptr && q_k != nullptr));
    return launch_reduce(ProjOp{z_k, r_k, p_k, q_k}, out2, ws, num_points, stream);
}

int fdd_dom_inner_product_flexible(double *out, double *ws, const double *r_k, const double *r_kp1, const double *z_k, int num_points, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && num_points >= 0);
    FDD_REQUIRE(num_points == 0 || (r_k != nullptr && r_kp1 != nullptr && z_k != nullptr));
    return launch_reduce(FlexOp{r_k, r_kp1, z_k}, out, ws, num_points, stream);
}

int fdd_dom_inner_product_flexible_gamma(double *out2, double *ws, const double *r_k, const double *r_kp1, const double *z_k, int num_points, void *stream)
{
    FDD_REQUIRE(out2 != nullptr && ws != nullptr && num_points >= 0);
    FDD_REQUIRE(num_points == 0 || (r_k != nullptr && r_kp1 != nullptr && z_k != nullptr));
    return launch_reduce(FlexGammaOp{r_k, r_kp1, z_k}, out2, ws, num_points, stream);
}

int fdd_dom_lincomb_flexible_gamma(double *out2, double *ws, const double *r_k, const double *r_kp1, double *z_k, int num_points, int slice_begin, int slice_size, int z_is_zero, const double *coeffs_dev, const double *const *v, const double *v_scale_dev, const double *last_dev, int m, void *stream)
{
    FDD_REQUIRE(out2 != nullptr && ws != nullptr && num_points >= 0 && m >= 1 && m <= FDD_MULTI_MAX);
    FDD_REQUIRE(slice_begin >= 0 && slice_size >= 0 && (long long)slice_begin + slice_size <= num_points);
    FDD_REQUIRE(num_points == 0 || (r_k != nullptr && r_kp1 != nullptr && z_k != nullptr));
    FDD_REQUIRE(slice_size == 0 || (coeffs_dev != nullptr && v != nullptr));
    if (slice_size == 0) return launch_reduce(FlexGammaOp{r_k, r_kp1, z_k}, out2, ws, num_points, stream);
    for (int k = 0; k < m; k++) FDD_REQUIRE(v[k] != nullptr && v[k] != z_k + slice_begin);
    const bool zero = z_is_zero != 0;
    switch (m)
    {
    case 1: return launch_lincomb_flex_gamma<1>(out2, ws, r_k, r_kp1, z_k, num_points, slice_begin, slice_size, zero, coeffs_dev, v, v_scale_dev, last_dev, stream);
    case 2: return launch_lincomb_flex_gamma<2>(out2, ws, r_k, r_kp1, z_k, num_points, slice_begin, slice_size, zero, coeffs_dev, v, v_scale_dev, last_dev, stream);
    case 3: return launch_lincomb_flex_gamma<3>(out2, ws, r_k, r_kp1, z_k, num_points, slice_begin, slice_size, zero, coeffs_dev, v, v_scale_dev, last_dev, stream);
    case 4: return launch_lincomb_flex_gamma<4>(out2, ws, r_k, r_kp1, z_k, num_points, slice_begin, slice_size, zero, coeffs_dev, v, v_scale_dev, last_dev, stream);
    case 5: return launch_lincomb_flex_gamma<5>(out2, ws, r_k, r_kp1, z_k, num_points, slice_begin, slice_size, zero, coeffs_dev, v, v_scale_dev, last_dev, stream);
    case 6: return launch_lincomb_flex_gamma<6>(out2, ws, r_k, r_kp1, z_k, num_points, slice_begin, slice_size, zero, coeffs_dev, v, v_scale_dev, last_dev, stream);
    case 7: return launch_lincomb_flex_gamma<7>(out2, ws, r_k, r_kp1, z_k, num_points, slice_begin, slice_size, zero, coeffs_dev, v, v_scale_dev, last_dev, stream);
    default: return launch_lincomb_flex_gamma<8>(out2, ws, r_k, r_kp1, z_k, num_points, slice_begin, slice_size, zero, coeffs_dev, v, v_scale_dev, last_dev, stream);
    }
}

int fdd_dom_residual_update_norm2_dev(double *out, double *ws, double *r_kp1, const double *r_k, const double *q_k, const double *alpha_num, const double *alpha_den, int num_points, int slice_begin, int slice_size, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && num_points >= 0);
    FDD_REQUIRE(slice_begin >= 0 && slice_size >= 0 && (long long)slice_begin + slice_size <= num_points);
    FDD_REQUIRE(num_points == 0 || (r_kp1 != nullptr && r_k != nullptr && q_k != nullptr && alpha_num != nullptr && alpha_den != nullptr));
    hipStream_t s = fdd_stream(stream);
    const ResidualUpdateNormOp op{r_kp1, r_k, q_k, alpha_num, alpha_den};
    const long long lo = slice_begin, nd = slice_size, n = num_points;
    // the norm's own launch on r_kp1 + lo (launch_reduce): path, grid, and an empty sum as a cleared scalar
    const bool pairs = nd >= 2 && fdd_aligned(r_kp1 + lo, Pair::bytes<double>);
    const bool wide_loads = fdd_aligned(r_k + lo, Pair::bytes<double>) && fdd_aligned(q_k + lo, Pair::bytes<double>);
    if (nd == 0)
    {
        if (hipError_t e = hipMemsetAsync(out, 0, sizeof(double), s)) return (int)e;
        if (n == 0) return 0;
        hipLaunchKernelGGL(residual_update_norm_kernel<false>, dim3(fdd_stream_grid(n, kBlock)), dim3(kBlock), 0, s, op, ws, lo, nd, n, wide_loads);
        FDD_LAUNCH_CHECK();
        return 0;
    }
    const int grid = fdd_stream_grid(pairs ? nd / 2 : nd, kBlock);
    if (pairs)
        hipLaunchKernelGGL(residual_update_norm_kernel<true>, dim3(grid), dim3(kBlock), 0, s, op, ws, lo, nd, n, wide_loads);
    else
        hipLaunchKernelGGL(residual_update_norm_kernel<false>, dim3(grid), dim3(kBlock), 0, s, op, ws, lo, nd, n, wide_loads);
    FDD_LAUNCH_CHECK();
    hipLaunchKernelGGL(reduce_final_kernel<1>, dim3(1), dim3(kBlock), 0, s, out, ws, grid);
    FDD_LAUNCH_CHECK();
    return 0;
}

int fdd_sub_inner_product(double *out, double *ws, const double *u, const double *v, int num_values, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && num_values >= 0);
    FDD_REQUIRE(num_values == 0 || (u != nullptr && v != nullptr));
    return launch_reduce(Dot2Op{u, v}, out, ws, num_values, stream);
}

int fdd_sub_weighted_inner_product(double *out, double *ws, const double *u, const double *v, const double *w, int num_values, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && num_values >= 0);
    FDD_REQUIRE(num_values == 0 || (u != nullptr && v != nullptr && w != nullptr));
    return launch_reduce(Dot3Op{u, v, w}, out, ws, num_values, stream);
}

int fdd_sub_projection_inner_products(double *out2, double *ws, const double *z_k, const double *r_k, const double *p_k, const double *q_k, const double *weight, int num_values, void *stream)
{
    FDD_REQUIRE(out2 != nullptr && ws != nullptr && num_values >= 0);
    FDD_REQUIRE(num_values == 0 || (z_k != nullptr && r_k != nullptr && p_k != nullptr && q_k != nullptr && weight != nullptr));
    return launch_reduce(ProjWOp{z_k, r_k, p_k, q_k, weight}, out2, ws, num_values, stream);
}

int fdd_sub_search_update_inner_product(double *out, double *ws, const double *r_k, const double *r_kp1, const double *z_k, const double *weight, int num_points, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && num_points >= 0);
    FDD_REQUIRE(num_points == 0 || (r_k != nullptr && r_kp1 != nullptr && z_k != nullptr && weight != nullptr));
    return launch_reduce(FlexWOp{r_k, r_kp1, z_k, weight}, out, ws, num_points, stream);
}

int fdd_amg_dot(double *out, double *ws, const double *x, const double *y, int size, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && size >= 0);
    FDD_REQUIRE(size == 0 || (x != nullptr && y != nullptr));
    return launch_reduce(Dot2Op{x, y}, out, ws, size, stream);
}

int fdd_multi_weighted_inner_product(double *out, double *ws, const double *a, const double *const *b, int m, const double *w, int n, void *stream)
{
    return fdd_multi_weighted_inner_product_scaled(out, ws, a, b, nullptr, m, w, n, stream);
}

int fdd_multi_weighted_inner_product_scaled(double *out, double *ws, const double *a, const double *const *b, const double *b_scale_dev, int m, const double *w, int n, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && n >= 0 && m >= 1 && m <= FDD_MULTI_MAX && b != nullptr);
    FDD_REQUIRE(n == 0 || a != nullptr); // w == NULL: unit weights
    for (int k = 0; k < m; k++) FDD_REQUIRE(n == 0 || b[k] != nullptr);
    switch (m)
    {
    case 1: return launch_multi_dot<1>(out, ws, a, b, b_scale_dev, w, n, stream);
    case 2: return launch_multi_dot<2>(out, ws, a, b, b_scale_dev, w, n, stream);
    case 3: return launch_multi_dot<3>(out, ws, a, b, b_scale_dev, w, n, stream);
    case 4: return launch_multi_dot<4>(out, ws, a, b, b_scale_dev, w, n, stream);
    case 5: return launch_multi_dot<5>(out, ws, a, b, b_scale_dev, w, n, stream);
    case 6: return launch_multi_dot<6>(out, ws, a, b, b_scale_dev, w, n, stream);
    case 7: return launch_multi_dot<7>(out, ws, a, b, b_scale_dev, w, n, stream);
    default: return launch_multi_dot<8>(out, ws, a, b, b_scale_dev, w, n, stream);
    }
}

int fdd_multi_axpy_norm2_dev(double *out, double *ws, double *y, const double *coeffs_dev, double sign, const double *const *x, int m, const double *w, int n, void *stream)
{
    return fdd_multi_axpy_norm2_scaled_dev(out, ws, y, y, coeffs_dev, sign, x, nullptr, m, w, n, stream);
}

int fdd_multi_axpy_norm2_scaled_dev(double *out, double *ws, double *dst, const double *y, const double *coeffs_dev, double sign, const double *const *x, const double *x_scale_dev, int m, const double *w, int n, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && n >= 0 && m >= 1 && m <= FDD_MULTI_MAX && x != nullptr && coeffs_dev != nullptr);
    FDD_REQUIRE(n == 0 || y != nullptr); // w == NULL: unit weights; dst == NULL: the updated vector is not stored, only its norm formed
    for (int k = 0; k < m; k++) FDD_REQUIRE(n == 0 || x[k] != nullptr);
    switch (m)
    {
    case 1: return launch_multi_axpy_norm<1>(out, ws, dst, y, coeffs_dev, sign, x, x_scale_dev, w, n, stream);
    case 2: return launch_multi_axpy_norm<2>(out, ws, dst, y, coeffs_dev, sign, x, x_scale_dev, w, n, stream);
    case 3: return launch_multi_axpy_norm<3>(out, ws, dst, y, coeffs_dev, sign, x, x_scale_dev, w, n, stream);
    case 4: return launch_multi_axpy_norm<4>(out, ws, dst, y, coeffs_dev, sign, x, x_scale_dev, w, n, stream);
    case 5: return launch_multi_axpy_norm<5>(out, ws, dst, y, coeffs_dev, sign, x, x_scale_dev, w, n, stream);
    case 6: return launch_multi_axpy_norm<6>(out, ws, dst, y, coeffs_dev, sign, x, x_scale_dev, w, n, stream);
    case 7: return launch_multi_axpy_norm<7>(out, ws, dst, y, coeffs_dev, sign, x, x_scale_dev, w, n, stream);
    default: return launch_multi_axpy_norm<8>(out, ws, dst, y, coeffs_dev, sign, x, x_scale_dev, w, n, stream);
    }
}

// The two entries of an Arnoldi step whose vector is not read (the last of a cycle).  Double only: a float basis is orthogonal
// to about 1e-7, the identity behind fdd_norm_estimate.h does not hold to double rounding there, and the float inner solve
// keeps its pass and its bits.
int fdd_multi_weighted_inner_product_self(double *out, double *ws, const double *a, const double *const *b, const double *b_scale_dev, int m, const double *w, int n, void *stream)
{
    // one sum more than the m dots: the workspace and the fold hold FDD_MULTI_MAX of them
    FDD_REQUIRE(out != nullptr && ws != nullptr && n >= 0 && m >= 1 && m <= FDD_MULTI_MAX - 1 && b != nullptr);
    FDD_REQUIRE(n == 0 || a != nullptr); // w == NULL: unit weights
    for (int k = 0; k < m; k++) FDD_REQUIRE(n == 0 || b[k] != nullptr);
    int rc = 0;
    fdd_for_n<1, FDD_MULTI_MAX - 1>(m, [&](auto M) { rc = launch_multi_dot_self<M()>(out, ws, a, b, b_scale_dev, w, n, stream); });
    return rc;
}

int fdd_multi_axpy_norm2_scaled_gated_dev(double *out, double *ws, double *dst, const double *y, const double *coeffs_dev, double sign, const double *const *x, const double *x_scale_dev, int m, const double *w, int n, const double *dots_dev, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && n >= 0 && m >= 1 && m <= FDD_MULTI_MAX - 1 && x != nullptr && coeffs_dev != nullptr && dots_dev != nullptr);
    FDD_REQUIRE(n == 0 || y != nullptr); // w == NULL: unit weights; dst == NULL: only the norm is formed
    for (int k = 0; k < m; k++) FDD_REQUIRE(n == 0 || x[k] != nullptr);
    int rc = 0;
    fdd_for_n<1, FDD_MULTI_MAX - 1>(m, [&](auto M) { rc = launch_multi_axpy_norm<M()>(out, ws, dst, y, coeffs_dev, sign, x, x_scale_dev, w, n, stream, dots_dev); });
    return rc;
}

int fdd_gather_weighted_norm2(double *out, double *ws, const int *Qt_ptr, const int *Qt_col, const double *u, const double *node_weight, int num_nodes, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && num_nodes >= 0);
    hipStream_t s = fdd_stream(stream);
    if (num_nodes == 0) return (int)hipMemsetAsync(out, 0, sizeof(double), s);
    FDD_REQUIRE(Qt_ptr != nullptr && Qt_col != nullptr && u != nullptr && node_weight != nullptr);
    const int grid = fdd_stream_grid((num_nodes + 3) / 4, kBlock); // 4 nodes per lane per pass
    hipLaunchKernelGGL(gather_norm2_kernel, dim3(grid), dim3(kBlock), 0, s, ws, Qt_ptr, Qt_col, u, node_weight, num_nodes);
    FDD_LAUNCH_CHECK();
    hipLaunchKernelGGL(reduce_final_kernel<1>, dim3(1), dim3(kBlock), 0, s, out, ws, grid);
    FDD_LAUNCH_CHECK();
    return 0;
}

#define FDD_M_SWITCH(CALL)                                                          \
    switch (m)                                                                      \
    {                                                                               \
    case 1: return CALL(1);                                                         \
    case 2: return CALL(2);                                                         \
    case 3: return CALL(3);                                                         \
    case 4: return CALL(4);                                                         \
    case 5: return CALL(5);                                                         \
    case 6: return CALL(6);                                                         \
    case 7: return CALL(7);                                                         \
    case 8: return CALL(8);                                                         \
    default: fdd_set_error("at most 8 vectors per multi-vector reduction"); return FDD_ERR_INVALID_ARGUMENT; \
    }

int fdd_multi_inner_product_scaled_f32(double *out, double *ws, const float *a, const float *const *b, const double *b_scale_dev, int m, int n, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && m >= 1 && n >= 0);
    FDD_REQUIRE(n == 0 || (a != nullptr && b != nullptr));
#define FDD_CALL_DOT(M_) launch_multi_dot_f32<M_>(out, ws, a, b, b_scale_dev, n, stream)
    FDD_M_SWITCH(FDD_CALL_DOT)
#undef FDD_CALL_DOT
}

int fdd_multi_axpy_norm2_scaled_dev_f32(double *out, double *ws, float *dst, const float *y, const double *coeffs_dev, double sign, const float *const *x, const double *x_scale_dev, int m, int n, void *stream)
{
    FDD_REQUIRE(out != nullptr && ws != nullptr && m >= 1 && n >= 0);
    FDD_REQUIRE(n == 0 || (y != nullptr && x != nullptr && coeffs_dev != nullptr)); // dst == NULL: norm only
#define FDD_CALL_AN(M_) launch_multi_axpy_norm_f32<M_>(out, ws, dst, y, coeffs_dev, sign, x, x_scale_dev, n, stream)
    FDD_M_SWITCH(FDD_CALL_AN)
#undef FDD_CALL_AN
}
#undef FDD_M_SWITCH

} // extern "C"
