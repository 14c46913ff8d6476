// Successive-right-hand-side projection (an addition of this build; the reference has no counterpart): the three
// passes outside the Krylov solve when the outer solve starts from the A-norm best approximation in the span of
// earlier solutions.  The basis X and its images AX are one slab each, `capacity` rows of `ld` doubles (ld even, base
// 16-byte aligned, so every row takes 16-byte loads), and the kernels take (base, ld, K), K <= FDD_PROJECTION_MAX:
//
//   dots   out[k] = <X_k, f> for all K in one pass over f                       (K + 1 streams read)
//   apply  x = x_in + sign_x sum c_k X_k,  b = b_in + sign_b sum c_k AX_k, and
//          optionally <x, b> of the values just formed                          (2K + 2 streams read, 2 written)
//   store  X_k = x / sqrt(nu2), AX_k = b / sqrt(nu2), nu2 in device memory      (2 read, 2 written)
//
// All are HBM-bound with no reuse: the shape is fdd_reduce.hip's -- a capped grid striding over pairs with 16-byte
// non-temporal loads, private sums per lane, a wavefront __shfl_down tree, one partial per workgroup and value, and
// one final workgroup.  Results are deterministic for given n and K (fixed grid, fixed tree).  The workspace is the
// common one of fdd_reduce_workspace_doubles(): the dots' grid is capped so that K * grid partials fit in it.
#include "fdd_stream.h"

namespace
{

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / FDD_WAVE;
constexpr int kWsDoubles = FDD_MULTI_MAX * FDD_REDUCE_MAX_BLOCKS; // fdd_reduce_workspace_doubles()

__device__ __forceinline__ double ld1(const double *p, long long i) { return __builtin_nontemporal_load(p + i); }

// one partial per workgroup and value: ws[k * gridDim.x + blockIdx.x]
template <int NV>
__device__ __forceinline__ void block_reduce_store(const double (&a)[NV], double *ws)
{
    __shared__ double s[NV][kWaves];
    const int lane = threadIdx.x & (FDD_WAVE - 1);
    const int wave = threadIdx.x / FDD_WAVE;
#pragma unroll
    for (int k = 0; k < NV; k++)
    {
        const double x = wave_sum(a[k]);
        if (lane == 0) s[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < NV)
    {
        double x = s[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < kWaves; w++) x += s[threadIdx.x][w];
        ws[(long long)threadIdx.x * gridDim.x + blockIdx.x] = x;
    }
}

// second stage, one workgroup: value k is folded by wave k % kWaves, every lane adding its partials in block order
__global__ __launch_bounds__(kBlock) void projection_final_kernel(double *out, const double *ws, int nblocks, int nv)
{
    const int lane = threadIdx.x & (FDD_WAVE - 1);
    const int wave = threadIdx.x / FDD_WAVE;
    for (int k = wave; k < nv; k += kWaves)
    {
        double x = 0.0;
        for (int b = lane; b < nblocks; b += FDD_WAVE) x += ws[(long long)k * nblocks + b];
        x = wave_sum(x);
        if (lane == 0) out[k] = x;
    }
}

// PAIRS: f is 16-byte aligned and the lanes walk pairs (the slab rows always are); otherwise one value per lane
template <int K, bool PAIRS>
__global__ __launch_bounds__(kBlock) void projection_dots_kernel(double *ws, const double *X, long long ld, const double *f, long long n)
{
    double a[K];
#pragma unroll
    for (int k = 0; k < K; k++) a[k] = 0.0;

    const long long stride = (long long)gridDim.x * kBlock;
    const long long first = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (PAIRS)
    {
        const long long n2 = n / 2;
        for (long long i = first; i < n2; i += stride)
        {
            const double2 ff = ld2(f, i);
            double2 xx[K];
#pragma unroll
            for (int k = 0; k < K; k++) xx[k] = ld2(X + k * ld, i); // all K loads in flight before the first product
#pragma unroll
            for (int k = 0; k < K; k++)
            {
                a[k] += xx[k].x * ff.x;
                a[k] += xx[k].y * ff.y;
            }
        }
        if ((n & 1) && first == 0)
        {
#pragma unroll
            for (int k = 0; k < K; k++) a[k] += X[k * ld + n - 1] * f[n - 1];
        }
    }
    else
    {
        for (long long i = first; i < n; i += stride)
        {
            const double fi = ld1(f, i);
            double xx[K];
#pragma unroll
            for (int k = 0; k < K; k++) xx[k] = ld1(X + k * ld, i);
#pragma unroll
            for (int k = 0; k < K; k++) a[k] += xx[k] * fi;
        }
    }
    block_reduce_store<K>(a, ws);
}

// x = (x_in or 0) + sign_x sum c_k X_k, b = b_in + sign_b sum c_k AX_k, in the order k = 0 .. K - 1 (the statement of
// fdd_multi_axpy_dev on either vector); DOT: the product of the two values just formed enters <x, b> without a trip
// through memory.  x_in == x / b_in == b: every lane reads its own entries before it writes them.
template <int K, bool PAIRS, bool DOT>
__global__ __launch_bounds__(kBlock) void projection_apply_kernel(double *x, double *b, double *ws, const double *x_in, const double *b_in, const double *X, const double *AX, long long ld,
                                                                  const double *c, double sign_x, double sign_b, long long n)
{
    double cx[K > 0 ? K : 1], cb[K > 0 ? K : 1];
#pragma unroll
    for (int k = 0; k < K; k++)
    {
        const double ck = c[k];
        cx[k] = sign_x * ck;
        cb[k] = sign_b * ck;
    }
    double acc[1] = {0.0};

    auto one = [&](long long i) {
        double xv = x_in ? ld1(x_in, i) : 0.0, bv = ld1(b_in, i);
#pragma unroll
        for (int k = 0; k < K; k++)
        {
            xv = 1.0 * xv + cx[k] * ld1(X + k * ld, i);
            bv = 1.0 * bv + cb[k] * ld1(AX + k * ld, i);
        }
        x[i] = xv;
        b[i] = bv;
        if (DOT) acc[0] += xv * bv;
    };

    const long long stride = (long long)gridDim.x * kBlock;
    const long long first = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (PAIRS)
    {
        const long long n2 = n / 2;
        for (long long i = first; i < n2; i += stride)
        {
            double2 xv = x_in ? ld2(x_in, i) : make_double2(0.0, 0.0), bv = ld2(b_in, i);
            double2 xx[K > 0 ? K : 1], aa[K > 0 ? K : 1];
#pragma unroll
            for (int k = 0; k < K; k++)
            {
                xx[k] = ld2(X + k * ld, i);
                aa[k] = ld2(AX + k * ld, i);
            }
#pragma unroll
            for (int k = 0; k < K; k++)
            {
                xv.x = 1.0 * xv.x + cx[k] * xx[k].x;
                xv.y = 1.0 * xv.y + cx[k] * xx[k].y;
                bv.x = 1.0 * bv.x + cb[k] * aa[k].x;
                bv.y = 1.0 * bv.y + cb[k] * aa[k].y;
            }
            // default policy: the solver (x, b) or the next pass of the update reads them next
            reinterpret_cast<double2 *>(x)[i] = xv;
            reinterpret_cast<double2 *>(b)[i] = bv;
            if (DOT)
            {
                acc[0] += xv.x * bv.x;
                acc[0] += xv.y * bv.y;
            }
        }
        if ((n & 1) && first == 0) one(n - 1);
    }
    else
    {
        for (long long i = first; i < n; i += stride) one(i);
    }
    if (DOT) block_reduce_store<1>(acc, ws);
}

template <bool PAIRS>
__global__ __launch_bounds__(kBlock) void projection_store_kernel(double *Xk, double *AXk, const double *x, const double *b, const double *nu2, long long n)
{
    const double inv = 1.0 / sqrt(*nu2); // the factor of fdd_vector_scaling_rsqrt_dev
    const long long stride = (long long)gridDim.x * kBlock;
    const long long first = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (PAIRS)
    {
        const long long n2 = n / 2;
        for (long long i = first; i < n2; i += stride)
        {
            const double2 xv = ld2(x, i), bv = ld2(b, i);
            reinterpret_cast<double2 *>(Xk)[i] = make_double2(inv * xv.x, inv * xv.y);
            reinterpret_cast<double2 *>(AXk)[i] = make_double2(inv * bv.x, inv * bv.y);
        }
        if ((n & 1) && first == 0)
        {
            Xk[n - 1] = inv * x[n - 1];
            AXk[n - 1] = inv * b[n - 1];
        }
    }
    else
    {
        for (long long i = first; i < n; i += stride)
        {
            Xk[i] = inv * ld1(x, i);
            AXk[i] = inv * ld1(b, i);
        }
    }
}

template <int K>
int launch_dots(double *out, double *ws, const double *X, int ld, const double *f, int n, hipStream_t s)
{
    const bool pairs = fdd_aligned16(f) && n >= 2;
    // K * grid partials must fit the common workspace
    const int grid = fdd_stream_grid(pairs ? n / 2 : n, kBlock, kWsDoubles / K < FDD_REDUCE_MAX_BLOCKS ? kWsDoubles / K : FDD_REDUCE_MAX_BLOCKS);
    if (pairs)
        hipLaunchKernelGGL((projection_dots_kernel<K, true>), dim3(grid), dim3(kBlock), 0, s, ws, X, (long long)ld, f, (long long)n);
    else
        hipLaunchKernelGGL((projection_dots_kernel<K, false>), dim3(grid), dim3(kBlock), 0, s, ws, X, (long long)ld, f, (long long)n);
    FDD_LAUNCH_CHECK();
    hipLaunchKernelGGL(projection_final_kernel, dim3(1), dim3(kBlock), 0, s, out, ws, grid, K);
    FDD_LAUNCH_CHECK();
    return 0;
}

template <int K, bool DOT>
int launch_apply(double *x, double *b, double *nu2_out, double *ws, const double *x_in, const double *b_in, const double *X, const double *AX, int ld, const double *c, double sign_x, double sign_b, int n, hipStream_t s)
{
    const bool pairs = n >= 2 && fdd_aligned16(x) && fdd_aligned16(b) && fdd_aligned16(x_in) && fdd_aligned16(b_in); // NULL counts as aligned
    const int grid = fdd_stream_grid(pairs ? n / 2 : n, kBlock);
    if (pairs)
        hipLaunchKernelGGL((projection_apply_kernel<K, true, DOT>), dim3(grid), dim3(kBlock), 0, s, x, b, ws, x_in, b_in, X, AX, (long long)ld, c, sign_x, sign_b, (long long)n);
    else
        hipLaunchKernelGGL((projection_apply_kernel<K, false, DOT>), dim3(grid), dim3(kBlock), 0, s, x, b, ws, x_in, b_in, X, AX, (long long)ld, c, sign_x, sign_b, (long long)n);
    FDD_LAUNCH_CHECK();
    if (DOT)
    {
        hipLaunchKernelGGL(projection_final_kernel, dim3(1), dim3(kBlock), 0, s, nu2_out, ws, grid, 1);
        FDD_LAUNCH_CHECK();
    }
    return 0;
}

#define FDD_K_SWITCH(CALL)        \
    switch (K)                    \
    {                             \
    case 1: return CALL(1);       \
    case 2: return CALL(2);       \
    case 3: return CALL(3);       \
    case 4: return CALL(4);       \
    case 5: return CALL(5);       \
    case 6: return CALL(6);       \
    case 7: return CALL(7);       \
    case 8: return CALL(8);       \
    case 9: return CALL(9);       \
    case 10: return CALL(10);     \
    case 11: return CALL(11);     \
    case 12: return CALL(12);     \
    case 13: return CALL(13);     \
    case 14: return CALL(14);     \
    case 15: return CALL(15);     \
    default: return CALL(16);     \
    }

// the slab: K rows of ld doubles holding vectors of n
#define FDD_REQUIRE_SLAB(base)                                                    \
    FDD_REQUIRE(K >= 0 && K <= FDD_PROJECTION_MAX && n >= 0 && ld >= n && (ld & 1) == 0); \
    FDD_REQUIRE(K == 0 || n == 0 || ((base) != nullptr && fdd_aligned16(base)))

} // namespace

extern "C" {

int fdd_projection_dots(double *out, double *ws, const double *X, int ld, int K, const double *f, int n, void *stream)
{
    FDD_REQUIRE_SLAB(X);
    if (K == 0) return 0; // nothing to write
    FDD_REQUIRE(out != nullptr && ws != nullptr);
    hipStream_t s = fdd_stream(stream);
    if (n == 0) return (int)hipMemsetAsync(out, 0, sizeof(double) * K, s);
    FDD_REQUIRE(f != nullptr);
#define FDD_CALL_DOTS(K_) launch_dots<K_>(out, ws, X, ld, f, n, s)
    FDD_K_SWITCH(FDD_CALL_DOTS)
#undef FDD_CALL_DOTS
}

int fdd_projection_apply(double *x, double *b, double *nu2_out, double *ws, const double *x_in, const double *b_in, const double *X, const double *AX, int ld, int K, const double *coeffs_dev, double sign_x, double sign_b, int n, void *stream)
{
    FDD_REQUIRE_SLAB(X);
    FDD_REQUIRE(K == 0 || n == 0 || (AX != nullptr && fdd_aligned16(AX) && coeffs_dev != nullptr));
    FDD_REQUIRE(nu2_out == nullptr || ws != nullptr);
    hipStream_t s = fdd_stream(stream);
    if (n == 0) return nu2_out ? (int)hipMemsetAsync(nu2_out, 0, sizeof(double), s) : 0;
    FDD_REQUIRE(x != nullptr && b != nullptr && b_in != nullptr); // x_in == NULL: taken as 0, not read
    if (nu2_out)
    {
#define FDD_CALL_APPLY(K_) launch_apply<K_, true>(x, b, nu2_out, ws, x_in, b_in, X, AX, ld, coeffs_dev, sign_x, sign_b, n, s)
        if (K == 0) return FDD_CALL_APPLY(0);
        FDD_K_SWITCH(FDD_CALL_APPLY)
#undef FDD_CALL_APPLY
    }
#define FDD_CALL_APPLY(K_) launch_apply<K_, false>(x, b, nullptr, ws, x_in, b_in, X, AX, ld, coeffs_dev, sign_x, sign_b, n, s)
    if (K == 0) return FDD_CALL_APPLY(0);
    FDD_K_SWITCH(FDD_CALL_APPLY)
#undef FDD_CALL_APPLY
}

int fdd_projection_store(double *Xk, double *AXk, const double *x, const double *b, const double *nu2_dev, int n, void *stream)
{
    FDD_REQUIRE(n >= 0);
    if (n == 0) return 0;
    FDD_REQUIRE(Xk != nullptr && AXk != nullptr && x != nullptr && b != nullptr && nu2_dev != nullptr);
    hipStream_t s = fdd_stream(stream);
    const bool pairs = n >= 2 && fdd_aligned16(Xk) && fdd_aligned16(AXk) && fdd_aligned16(x) && fdd_aligned16(b);
    const int grid = fdd_stream_grid(pairs ? n / 2 : n, kBlock);
    if (pairs)
        hipLaunchKernelGGL(projection_store_kernel<true>, dim3(grid), dim3(kBlock), 0, s, Xk, AXk, x, b, nu2_dev, (long long)n);
    else
        hipLaunchKernelGGL(projection_store_kernel<false>, dim3(grid), dim3(kBlock), 0, s, Xk, AXk, x, b, nu2_dev, (long long)n);
    FDD_LAUNCH_CHECK();
    return 0;
}

} // extern "C"
